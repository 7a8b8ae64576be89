// tests/san/record_stub.cpp — TEST INFRASTRUCTURE ONLY: a host-memory stand-in for the launcher of
// record.hip, for the CPU build of engine.cpp + record.cpp over the stub runtime (hip_stub.cpp, where
// a "device" pointer is a host pointer). Like store_stub.cpp it really does the work (the recording
// items, their metadata and commands, byte by byte), sequentially and with the device form's
// treatment of faulty items, so the driver can compare what comes back through the staging of the
// host form with what it expects. It reads every input byte the kernels may read, writes exactly the
// extents the kernels may write and scribbles over the scratch it was promised, so a slot or a
// scratch size that is too small faults under ASan or shows in the results.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../minpaxos_amd/csrc/kernels.hpp"

namespace mpx {

uint64_t record_work_bytes(uint64_t n, Carver&& c) {
    (void)c.take<char>(16 * n + 16);
    (void)c.take<char>(n / 64 + 64);
    return c.bytes();
}

namespace {
unsigned touch(const void* p, uint64_t bytes) {
    unsigned sum = 0;
    for (uint64_t i = 0; i < bytes; ++i) sum += ((const uint8_t*)p)[i];
    return sum;
}
void put32(std::vector<uint8_t>& w, uint32_t x) {
    for (int k = 0; k < 4; ++k) w.push_back((uint8_t)(x >> (8 * k)));
}
void put64(std::vector<uint8_t>& w, uint64_t x) {
    for (int k = 0; k < 8; ++k) w.push_back((uint8_t)(x >> (8 * k)));
}
}  // namespace

hipError_t launch_record_log(const mpx_record_batch* b, uint8_t* out, uint64_t out_cap, uint64_t* item_off,
                             mpx_record_result* res, void* work, uint64_t work_bytes, uint32_t* err,
                             hipStream_t) {
    const uint64_t n = b->n;
    if (n >= 0xFFFFFFFFull || b->n_src > MPX_SC_MAX_SRC || b->kind > MPX_LR_DECIDED) return hipErrorInvalidValue;
    const size_t n_src = b->kind == MPX_LR_DECIDED ? 0 : b->n_src;
    const bool msgs = b->kind <= MPX_LR_COMMITS;
    uint64_t cmds = 0, rec_end[MPX_SC_MAX_SRC], recs = 0;
    unsigned sum = 0;
    for (size_t s = 0; s < n_src; ++s) {
        const mpx_store_src& x = b->src[s];
        cmds += x.n_cmds, rec_end[s] = recs += x.n_recs;
        // every byte of the sources is read (a staging slot that is too small faults here)
        sum += touch(x.op, x.n_cmds) + touch(x.key, 8 * x.n_cmds) + touch(x.val, 8 * x.n_cmds);
        if (x.n_frames) sum += touch(x.cmd_off, 8 * (x.n_frames + 1));
    }
    const bool one = (!(b->flags & MPX_LR_GENERAL) && n <= MPX_LR_ONE_LAUNCH_ITEMS &&
                      cmds <= MPX_LR_ONE_LAUNCH_CMDS) || !n;
    if (!one) {
        const uint64_t need = record_work_bytes(n);
        if (work_bytes < need) return hipErrorInvalidValue;
        memset(work, 0xEE, need);
    }
    const uint64_t n_eff = b->d_n ? std::min<uint64_t>(*b->d_n, n) : n;
    sum += touch(b->items, n_eff * (msgs ? sizeof(mpx_accept_msg) : sizeof(mpx_accept_send)));
    if (msgs) sum += touch(b->effect, n_eff);
    if (msgs && b->perm) sum += touch(b->perm, 4 * n_eff);
    const uint32_t status = b->kind == MPX_LR_ACCEPTS ? MPX_ACCEPTED : b->kind == MPX_LR_SENDS ? MPX_PREPARED : MPX_COMMITTED;
    std::vector<uint8_t> w;
    std::vector<uint64_t> off(n + 1, 0);
    uint64_t n_recs = 0, n_cmds = 0;
    for (uint64_t i = 0; i < n; ++i) {
        off[i] = w.size();
        if (i >= n_eff) continue;
        int32_t instance, ballot;
        uint64_t lo = 0, len = 0;
        size_t sid = 0;
        if (msgs) {
            const mpx_accept_msg& m = ((const mpx_accept_msg*)b->items)[i];
            instance = m.instance, ballot = m.ballot;
            bool with = true;
            if (b->kind == MPX_LR_ACCEPTS) {
                if (!(b->effect[i] & MPX_AH_STORED)) continue;
            } else {
                with = (b->effect[i] & MPX_CH_CMDS) && m.value_id != MPX_VALUE_KEEP;
            }
            if (with) {
                const uint64_t p = b->perm ? b->perm[i] : i;
                if (p >= recs) {
                    *err |= kErrInval;
                    continue;
                }
                while (sid + 1 < n_src && p >= rec_end[sid]) ++sid;
                const mpx_store_src& x = b->src[sid];
                if (m.value_id >= x.n_frames) {
                    *err |= kErrInval;
                    continue;
                }
                lo = x.cmd_off[m.value_id];
                const uint64_t hi = x.cmd_off[m.value_id + 1];
                if (hi < lo || hi > x.n_cmds || hi - lo >= 0xFFFFFFFFull) {
                    *err |= kErrInval;
                    continue;
                }
                len = hi - lo;
            }
        } else {
            const mpx_accept_send& x = ((const mpx_accept_send*)b->items)[i];
            instance = x.instance, ballot = x.ballot;
            if (!(x.flags & MPX_PH_ACCEPT)) continue;
            if (b->kind == MPX_LR_SENDS) {
                lo = x.first_cmd, len = x.n_cmds;
                if (lo > b->src[0].n_cmds || len > b->src[0].n_cmds - lo || len == 0xFFFFFFFFull) {
                    *err |= kErrInval;
                    continue;
                }
            } else {
                const int64_t rel = (int64_t)instance - b->inst_base;
                if (rel < 0 || (uint64_t)rel >= b->n_inst) {
                    *err |= kErrNil;
                    continue;
                }
                if (!b->mask[rel]) continue;
            }
        }
        put32(w, (uint32_t)ballot);
        if (b->format == MPX_LOG_DURABLE) put32(w, status), put32(w, (uint32_t)instance);
        else w.push_back((uint8_t)status);
        for (uint64_t j = 0; j < len; ++j) {
            const mpx_store_src& x = b->src[sid];
            w.push_back(x.op[lo + j]);
            put64(w, (uint64_t)x.key[lo + j]);
            put64(w, (uint64_t)x.val[lo + j]);
        }
        ++n_recs, n_cmds += len;
    }
    off[n] = w.size();
    const bool full = w.size() > out_cap;
    *res = mpx_record_result{n_recs, n_cmds, w.size() + (sum & 0u), full ? (uint64_t)MPX_LR_FULL : 0};
    if (item_off) memcpy(item_off, off.data(), (n + 1) * sizeof(uint64_t));
    if (!full && !w.empty()) memcpy(out, w.data(), w.size());
    return hipSuccess;
}

}  // namespace mpx

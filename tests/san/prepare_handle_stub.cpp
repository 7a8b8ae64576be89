// tests/san/prepare_handle_stub.cpp — TEST INFRASTRUCTURE ONLY: host-memory stand-ins for the
// launchers of prepare_handle.hip, for the CPU build of engine.cpp + prepare_handle.cpp over the
// stub runtime (hip_stub.cpp, where a "device" pointer is a host pointer). Like
// accepts_stored_stub.cpp they really do the work: the gather, both handlePrepares and the
// PrepareReply Marshals, with the device forms' treatment of faults (the error word, a reply
// that encodes as empty), so the driver can compare what comes back through the staging of the
// host forms with bytes worked by hand. They read the whole of every staged array, write exactly
// the extents the kernels may write and scribble over the scratch they were promised. What they
// were handed is left in ph_stub_seen for the driver.
#include <cstring>
#include <vector>

#include "../../minpaxos_amd/csrc/kernels.hpp"

struct PhStubSeen {
    uint64_t calls, n_src, n_inst, non_nil, flagged, n_groups;
};
PhStubSeen ph_stub_seen;

namespace mpx {

uint64_t prepare_replies_work_bytes(uint32_t n_dest, uint64_t n, uint64_t n_inst, Carver&& c) {
    (void)c.take<uint64_t>(n_inst + 1);
    (void)c.take<uint64_t>(n_inst + 1);
    (void)c.take<uint64_t>((uint64_t)n_dest * n + 1);
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
void put_varint(std::vector<uint8_t>& w, uint64_t n) {  // binary.PutVarint of n >= 0
    uint64_t u = n << 1;
    while (u >= 0x80) w.push_back((uint8_t)(u | 0x80)), u >>= 7;
    w.push_back((uint8_t)u);
}
void put_cmd(std::vector<uint8_t>& w, uint8_t op, int64_t k, int64_t v) {
    w.push_back(op), put64(w, (uint64_t)k), put64(w, (uint64_t)v);
}
int32_t get32(const uint8_t* p) {
    uint32_t x;
    memcpy(&x, p, 4);
    return (int32_t)x;
}
volatile unsigned g_sum;
}  // namespace

hipError_t launch_gather_prepares(int mode, const uint8_t* buf, uint64_t len,
                                  const mpx_peer_frame* other, uint64_t n_other,
                                  const uint64_t* d_n_other, int32_t group, mpx_prepare_msg* msgs,
                                  uint32_t* frame_index, uint64_t cap, uint64_t* n_prepares,
                                  void* work, uint64_t work_bytes, uint32_t* err, hipStream_t) {
    if (n_other) {
        if (work_bytes < prepare_replies_work_bytes(1, n_other, 0)) return hipErrorInvalidValue;
        memset(work, 0xEE, prepare_replies_work_bytes(1, n_other, 0));
    }
    g_sum = touch(buf, len) + touch(other, n_other * sizeof(mpx_peer_frame));
    const uint64_t lim = d_n_other && *d_n_other < n_other ? *d_n_other : n_other;
    const uint64_t body = mode == MPX_MODE_MIN ? 12 : 13;
    uint64_t k = 0;
    for (uint64_t i = 0; i < lim; ++i) {
        if (other[i].code != MPX_PEER_PREPARE) continue;
        const uint64_t slot = k++;
        if (slot >= cap) continue;
        const uint64_t p = (uint64_t)other[i].offset + 1;
        if (p + body > len) {
            *err |= kErrInval;
            continue;
        }
        if (mode == MPX_MODE_MIN)
            msgs[slot] = {group, get32(buf + p + 4), get32(buf + p), get32(buf + p + 8)};
        else
            msgs[slot] = {get32(buf + p + 4), get32(buf + p + 8), get32(buf + p), buf[p + 12]};
        frame_index[slot] = (uint32_t)i;
    }
    *n_prepares = k;
    return hipSuccess;
}

hipError_t launch_prepare_handle(int mode, const mpx_prepare_msg* msgs, uint64_t n,
                                 const mpx_acceptor_state* st, uint64_t n_inst, int32_t base,
                                 mpx_proposer_group* groups, uint64_t n_groups, uint32_t ipg,
                                 int32_t nrep, mpx_group_prep_state* gps, int32_t* pc,
                                 void* replies, int32_t* reply_to, uint8_t* effect,
                                 int32_t* log_from, uint32_t* err, hipStream_t) {
    const bool min = mode == MPX_MODE_MIN;
    g_sum = touch(msgs, n * sizeof(*msgs)) + touch(st, n_inst * sizeof(*st)) +
            touch(groups, n_groups * sizeof(*groups)) +
            (gps ? touch(gps, n_groups * sizeof(*gps)) : 0) +
            (pc ? touch(pc, n_groups * (uint64_t)nrep * 4) : 0);
    ++ph_stub_seen.calls;
    ph_stub_seen.n_inst = n_inst, ph_stub_seen.n_groups = n_groups;
    auto* rm = (mpx_prepare_reply_min*)replies;
    auto* rc = (mpx_prepare_reply*)replies;
    std::vector<bool> dead(n_groups, false);
    for (uint64_t i = 0; i < n; ++i) {
        const mpx_prepare_msg& m = msgs[i];
        if (i && msgs[i - 1].key > m.key) *err |= kErrOrder;
        if (m.leader_id < 0 || m.leader_id >= nrep) *err |= kErrBadId;
        reply_to[i] = m.leader_id;
        effect[i] = 0;
        const int64_t idx = (int64_t)m.key - base;
        if (min ? (m.key < 0 || (uint64_t)m.key >= n_groups) : (idx < 0 || (uint64_t)idx >= n_inst)) {
            *err |= min ? kErrInval : kErrNil;
            if (min) rm[i] = {0, 0, 0, 0, 0, MPX_VALUE_KEEP}, log_from[i] = 1;
            else rc[i] = {m.key, 0, 0, MPX_VALUE_KEEP};
            continue;
        }
        if (!min) {
            mpx_proposer_group& g = groups[(uint64_t)idx / ipg];
            const mpx_acceptor_state& s = st[idx];
            if (s.status == MPX_STATUS_NIL)
                rc[i] = {m.key, g.default_ballot, g.default_ballot > m.ballot ? 0u : 1u, MPX_VALUE_KEEP};
            else
                rc[i] = {m.key, s.ballot, m.ballot < s.ballot ? 0u : 1u, (uint32_t)idx};
            effect[i] = rc[i].ok ? MPX_PRH_OK : 0;
            if (m.arg == 1 && m.ballot > g.default_ballot)
                g.default_ballot = m.ballot, effect[i] |= MPX_PRH_RAISED;
            continue;
        }
        mpx_proposer_group& g = groups[m.key];
        const int64_t first = (int64_t)base + (int64_t)m.key * ipg, endw = first + ipg;
        uint32_t eff = 0;
        if (g.default_ballot < m.ballot) {
            eff = MPX_PRH_OK | MPX_PRH_RAISED;
            g.default_ballot = m.ballot, g.leader = m.leader_id, g.prepare_oks = 0;
            if (gps) {
                mpx_group_prep_state& p = gps[m.key];
                p.default_ballot = m.ballot, p.prepare_oks = 0, p.nacks = 0;
                p.max_recv_ballot = m.ballot, p.highest_instance = (int32_t)first;
                p.value_id = MPX_VALUE_KEEP;
            }
            if (pc)
                for (int32_t q = 0; q < nrep; ++q) pc[(uint64_t)m.key * nrep + q] = (int32_t)first;
        }
        int64_t crt = g.crt_instance;
        while (!dead[m.key]) {
            if (crt < first || crt >= endw) {
                dead[m.key] = true;
                break;
            }
            if (st[crt - base].status == MPX_STATUS_NIL) break;
            ++crt;
        }
        g.crt_instance = (int32_t)crt;
        const int32_t cu = g.committed_upto;
        uint32_t vid = MPX_VALUE_KEEP;
        int32_t lf = cu + 1;
        if (dead[m.key]) {
            *err |= kErrNil;
        } else if (cu > m.arg) {
            bool bad = false;
            if (crt > cu) {
                const int64_t s = (int64_t)cu + 1;
                if (s < first || s >= endw || st[s - base].status == MPX_STATUS_NIL) bad = true;
                else vid = (uint32_t)(s - base);
            }
            const int64_t lo = (int64_t)m.arg + 1;
            if (lo < first || cu >= endw) bad = true;
            for (int64_t r = lo; !bad && r <= cu; ++r)
                if (st[r - base].status == MPX_STATUS_NIL) bad = true;
            if (bad) *err |= kErrNil, vid = MPX_VALUE_KEEP;
            else eff |= MPX_PRH_LOG, lf = (int32_t)lo;
        }
        rm[i] = {g.self_id, (int32_t)(crt - 1), g.default_ballot, cu, eff & MPX_PRH_OK, vid};
        log_from[i] = lf;
        effect[i] = (uint8_t)eff;
    }
    return hipSuccess;
}

hipError_t launch_encode_prepare_replies(int mode, const mpx_prepare_reply_batch* b, uint8_t* out,
                                         uint64_t out_cap, uint64_t* dest_off, void* work,
                                         uint64_t work_bytes, uint32_t* err, hipStream_t) {
    const bool min = mode == MPX_MODE_MIN;
    const uint64_t n_inst = b->n_inst;
    if (b->n) {
        const uint64_t need = prepare_replies_work_bytes(b->n_dest, b->n, n_inst);
        if (work_bytes < need) return hipErrorInvalidValue;
        memset(work, 0xEE, need);
    }
    const size_t rb = min ? sizeof(mpx_prepare_reply_min) : sizeof(mpx_prepare_reply);
    unsigned sum = touch(b->replies, b->n * rb) + touch(b->reply_to, b->n * 4);
    if (min) sum += touch(b->log_from, b->n * 4);
    if (b->st) sum += touch(b->st, n_inst * sizeof(mpx_acceptor_state));
    if (b->lb) sum += touch(b->lb, n_inst * sizeof(mpx_inst_state));
    if (b->inst) sum += touch(b->inst, n_inst * sizeof(mpx_inst_cmds));
    sum += touch(b->src_op, b->n_src) + touch(b->src_key, 8 * b->n_src) + touch(b->src_val, 8 * b->n_src);
    g_sum = sum;
    ++ph_stub_seen.calls;
    ph_stub_seen.n_src = b->n_src, ph_stub_seen.n_inst = n_inst;
    ph_stub_seen.non_nil = ph_stub_seen.flagged = 0;
    for (uint64_t i = 0; i < n_inst; ++i) {
        if (b->st) ph_stub_seen.non_nil += b->st[i].status != MPX_STATUS_NIL;
        if (b->inst) ph_stub_seen.flagged += (b->inst[i].flags & MPX_IC_HAS_CMDS) != 0;
    }
    auto cmds_of = [&](uint64_t i, bool& fault) -> uint64_t {  // the commands slot i marshals
        const mpx_inst_cmds& c = b->inst[i];
        if (!(c.flags & MPX_IC_HAS_CMDS)) return 0;
        if (c.first_cmd > b->n_src || c.n_cmds > b->n_src - c.first_cmd) {
            fault = true;
            return 0;
        }
        return c.n_cmds;
    };
    std::vector<uint8_t> w;
    for (uint32_t q = 0; q < b->n_dest; ++q) {
        dest_off[q] = w.size();
        for (uint64_t s = 0; s < b->n; ++s) {
            const int32_t to = b->reply_to[s];
            if (to < 0) continue;
            if ((uint32_t)to >= b->n_dest) {
                *err |= kErrInval;
                continue;
            }
            if ((uint32_t)to != q) continue;
            uint32_t vid, ok;
            int32_t lc = 0;
            w.push_back(MPX_PEER_PREPARE_REPLY);
            if (min) {
                const mpx_prepare_reply_min& r = ((const mpx_prepare_reply_min*)b->replies)[s];
                put32(w, (uint32_t)r.id), put32(w, (uint32_t)r.instance), w.push_back((uint8_t)r.ok);
                put32(w, (uint32_t)r.ballot), put32(w, (uint32_t)r.last_committed);
                vid = r.value_id, ok = r.ok, lc = r.last_committed;
            } else {
                const mpx_prepare_reply& r = ((const mpx_prepare_reply*)b->replies)[s];
                put32(w, (uint32_t)r.instance), w.push_back((uint8_t)r.ok), put32(w, (uint32_t)r.ballot);
                vid = r.value_id, ok = r.ok;
            }
            (void)ok;
            uint64_t nc = 0;
            if (vid != MPX_VALUE_KEEP) {
                bool fault = false;
                if (vid >= n_inst || !b->inst) fault = true;
                else nc = cmds_of(vid, fault);
                if (fault) *err |= kErrInval;
            }
            put_varint(w, nc);
            for (uint64_t j = 0; j < nc; ++j) {
                const uint64_t at = b->inst[vid].first_cmd + j;
                put_cmd(w, b->src_op[at], b->src_key[at], b->src_val[at]);
            }
            if (!min) continue;
            int64_t lo = (int64_t)b->log_from[s] - b->inst_base, hi = (int64_t)lc - b->inst_base;
            if (lo <= hi && (lo < 0 || (uint64_t)hi >= n_inst)) *err |= kErrInval, hi = lo - 1;
            put_varint(w, lo <= hi ? (uint64_t)(hi - lo + 1) : 0);
            for (int64_t i = lo; i <= hi; ++i) {
                int32_t status = b->st[i].status;
                if (b->lb && b->lb[i].status != MPX_STATUS_NIL) status = b->lb[i].status;
                bool fault = false;
                uint64_t k = cmds_of((uint64_t)i, fault);
                if (b->st[i].status == MPX_STATUS_NIL) *err |= kErrNil, k = 0;
                else if (fault) *err |= kErrInval;
                put32(w, (uint32_t)b->st[i].ballot), put32(w, (uint32_t)status);
                put_varint(w, k);
                for (uint64_t j = 0; j < k; ++j) {
                    const uint64_t at = b->inst[i].first_cmd + j;
                    put_cmd(w, b->src_op[at], b->src_key[at], b->src_val[at]);
                }
            }
        }
    }
    dest_off[b->n_dest] = w.size();
    const uint64_t n_out = w.size() < out_cap ? w.size() : out_cap;  // nothing at or past out_cap
    if (n_out) memcpy(out, w.data(), n_out);
    return hipSuccess;
}

}  // namespace mpx

// tests/san/accepts_stored_stub.cpp — TEST INFRASTRUCTURE ONLY: a host-memory stand-in for the
// launcher of accepts_stored.hip, for the CPU build of engine.cpp + accepts_stored.cpp over the stub
// runtime (hip_stub.cpp, where a "device" pointer is a host pointer). Like record_stub.cpp it really
// does the work: bcastAccept's ring walk and the Marshals, frame by frame, with the device form's
// treatment of a nil instance and of a range that leaves the arena (no commands, the error word),
// so the driver can compare what comes back through the staging of the host form with bytes worked
// by hand. It reads the whole of every staged array, writes exactly the extents the kernels may
// write and scribbles over the scratch it was promised. What it was handed is left in
// as_stub_seen for the driver: the staged arena's size and the non-nil slots of the staged window.
#include <cstring>
#include <vector>

#include "../../minpaxos_amd/csrc/kernels.hpp"

struct AsStubSeen {
    uint64_t calls, n_src, non_nil, flagged;
};
AsStubSeen as_stub_seen;

namespace mpx {

uint64_t accepts_stored_work_bytes(uint32_t nrep, uint64_t n_sends, uint64_t n_inst, Carver&& c) {
    (void)c.take<uint64_t>(n_inst + 1);
    (void)c.take<uint64_t>(n_inst + 1);
    (void)c.take<uint64_t>((uint64_t)nrep * n_sends + 1);
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
volatile unsigned g_sum;
}  // namespace

hipError_t launch_encode_accepts_stored(int mode, int32_t nrep, const mpx_accept_store_batch* b,
                                        uint8_t* out, uint64_t out_cap, uint64_t* dest_off,
                                        void* work, uint64_t work_bytes, uint32_t* err, hipStream_t) {
    const bool min = mode == MPX_MODE_MIN;
    const uint64_t n_inst = (uint64_t)b->n_groups * b->ipg;
    const int32_t N = nrep;
    if (b->n_sends) {
        if (work_bytes < accepts_stored_work_bytes((uint32_t)N, b->n_sends, n_inst))
            return hipErrorInvalidValue;
        memset(work, 0xEE, accepts_stored_work_bytes((uint32_t)N, b->n_sends, n_inst));
    }
    unsigned sum = touch(b->sends, b->n_sends * sizeof(mpx_accept_send));
    if (b->n_sends) sum += touch(b->groups, b->n_groups * sizeof(mpx_proposer_group));
    if (b->cmd_op) sum += touch(b->cmd_op, b->n_cmds);
    if (b->cmd_key) sum += touch(b->cmd_key, 8 * b->n_cmds);
    if (b->cmd_val) sum += touch(b->cmd_val, 8 * b->n_cmds);
    ++as_stub_seen.calls;
    if (min && b->n_sends) {
        sum += touch(b->peer_commits, b->n_groups * (uint64_t)N * 4);
        sum += touch(b->st, n_inst * sizeof(mpx_acceptor_state));
        sum += touch(b->inst, n_inst * sizeof(mpx_inst_cmds));
        sum += touch(b->src_op, b->n_src) + touch(b->src_key, 8 * b->n_src) +
               touch(b->src_val, 8 * b->n_src);
        as_stub_seen.n_src = b->n_src;
        as_stub_seen.non_nil = as_stub_seen.flagged = 0;
        for (uint64_t i = 0; i < n_inst; ++i) {
            as_stub_seen.non_nil += b->st[i].status != MPX_STATUS_NIL;
            as_stub_seen.flagged += (b->inst[i].flags & MPX_IC_HAS_CMDS) != 0;
        }
    }
    g_sum = sum;
    std::vector<uint8_t> w;
    for (int32_t q = 0; q < N; ++q) {
        dest_off[q] = w.size();
        for (uint64_t s = 0; s < b->n_sends; ++s) {
            const mpx_accept_send& x = b->sends[s];
            if (!(x.flags & MPX_PH_ACCEPT)) continue;
            const int64_t idx = (int64_t)x.instance - b->inst_base;
            if (idx < 0 || (uint64_t)idx >= n_inst) {
                *err |= kErrNil;
                continue;
            }
            const uint64_t g = (uint64_t)idx / b->ipg;
            const int32_t self = b->groups[g].self_id;
            if (self < 0 || self >= N) {
                *err |= kErrBadId;
                continue;
            }
            // the ring walk from self: is q among the first n successors (CLASSIC: alive ones)?
            bool dest = false;
            const int n = (b->flags & MPX_AB_THRIFTY) ? N >> 1 : N - 1;
            int32_t p = self;
            for (int sent = 0; sent < n;) {
                p = (p + 1) % N;
                if (p == self) break;
                if (!min && !((b->alive_mask >> p) & 1u)) continue;
                ++sent;
                if (p == q) dest = true;
            }
            if (!dest) continue;
            const int64_t first = (int64_t)(g * b->ipg), lc = (int64_t)x.last_committed - b->inst_base;
            if (min && (lc < first - 1 || lc >= idx)) {
                *err |= kErrInval;
                continue;
            }
            w.push_back(MPX_PEER_ACCEPT);
            put32(w, (uint32_t)self), put32(w, (uint32_t)x.instance), put32(w, (uint32_t)x.ballot);
            if (min) put32(w, (uint32_t)x.last_committed);
            put_varint(w, x.n_cmds);
            for (uint64_t j = x.first_cmd; j < x.first_cmd + x.n_cmds; ++j)
                put_cmd(w, b->cmd_op[j], b->cmd_key[j], b->cmd_val[j]);
            if (!min) continue;
            const int64_t pc = (int64_t)b->peer_commits[g * N + q] - b->inst_base;
            const int64_t lo = pc < first ? first : pc + 1;
            put_varint(w, lo <= lc ? (uint64_t)(lc - lo + 1) : 0);
            for (int64_t i = lo; i <= lc; ++i) {
                const mpx_inst_cmds& c = b->inst[i];
                int32_t status = b->st[i].status;
                if (b->lb && b->lb[i].status != MPX_STATUS_NIL) status = b->lb[i].status;
                uint64_t nc = (c.flags & MPX_IC_HAS_CMDS) ? c.n_cmds : 0;
                if (b->st[i].status == MPX_STATUS_NIL) *err |= kErrNil, nc = 0;
                else if ((c.flags & MPX_IC_HAS_CMDS) &&
                         (c.first_cmd > b->n_src || c.n_cmds > b->n_src - c.first_cmd))
                    *err |= kErrInval, nc = 0;
                put32(w, (uint32_t)b->st[i].ballot), put32(w, (uint32_t)status);
                put_varint(w, nc);
                for (uint64_t j = c.first_cmd; j < c.first_cmd + nc; ++j)
                    put_cmd(w, b->src_op[j], b->src_key[j], b->src_val[j]);
            }
        }
    }
    dest_off[N] = w.size();
    const uint64_t n_out = w.size() < out_cap ? w.size() : out_cap;  // nothing at or past out_cap
    if (n_out) memcpy(out, w.data(), n_out);
    return hipSuccess;
}

}  // namespace mpx

// accepts_stored.hip — MIN's Accept bytes with the CatchUpLog read from the instance store.
//
// mpx_encode_accepts_stored: the frames of proposer.hip's mpx_encode_accepts (bcastAccept ->
// SendMsg -> Accept.Marshal, minpaxosprotomarsh.go:425-468), byte for byte, where the catch-up
// log is not a dense window-ordered copy but the state the turn already keeps on the device: the
// acceptor window st (ballot, status), the leader bookkeeping window lb (status once the tally has
// committed) and mpx_inst_cmds {first_cmd, n_cmds, flags} per slot pointing into the append-only
// command arena, where ranges lie in batch order, may be dead, and may be shared by two slots.
// The dense encoder's prefix sums stay, as scratch:
//   1. a scan (scan.hpp) of every window slot's command count: the synthetic lcoff[]. A slot counts
//      no commands when it is unflagged (Cmds == nil marshals as V(0), :117-123), nil, or its range
//      leaves the arena, so the sizes and the emitted bytes agree and no load leaves [0, n_src)
//   2. a scan of the slots' encoded sizes 8 + V(nc) + 17 nc from lcoff: log_off[]
//      (two scans, not one over a 16-byte pair: scan.hpp's lanes exchange items as one 64-bit
//      shuffle and its sum tiles keep 4 x 1088 items in LDS, 68 KB for a pair)
//   3. k_as_sizes / the frame scan / k_as_emit: the dense encoder's sizing, window search and piece
//      dealing over those two arrays. Only the log source differs (StoreLog): a catch-up command
//      piece (record ra, position x) is loaded from src[inst[ra].first_cmd + x], and a record's
//      header takes its ballot from st and its status from lb where lb has one, else from st.
// Nothing is materialised: no gathered copy of a catch-up run exists at any point.
// CLASSIC frames carry no log: the launcher hands them to launch_encode_accepts.
// Every step, the Accept frame and the scratch are catchup.hpp's; here: the kernels by name and
// the launcher.
#include "common.hpp"
#include "catchup.hpp"
#include "kernels.hpp"
#include "scan.hpp"

namespace mpx {

namespace {
using AsArgs = AcceptArgs<StoreLog>;
}  // namespace

__global__ __launch_bounds__(kFrBlock) void k_as_sizes(AsArgs a, uint64_t n_items,
                                                       uint64_t* __restrict__ size, uint32_t* err) {
    catchup_sizes(AcceptPolicy<MPX_MODE_MIN, StoreLog>{a}, n_items, size, err);
}
__global__ __launch_bounds__(kFrBlock) void k_as_emit(AsArgs a, const uint64_t* __restrict__ frame_off,
                                                      uint64_t n_items, uint8_t* __restrict__ out,
                                                      uint64_t out_cap, uint32_t* err) {
    catchup_emit(AcceptPolicy<MPX_MODE_MIN, StoreLog>{a}, frame_off, n_items, out, out_cap, err);
}

uint64_t accepts_stored_work_bytes(uint32_t nrep, uint64_t n_sends, uint64_t n_inst, Carver&& c) {
    // (the dense encoder's regions and lcoff: a CLASSIC call runs as launch_encode_accepts in it)
    return CatchupWork(c, nrep, n_sends, n_inst, true), c.bytes();
}

hipError_t launch_encode_accepts_stored(int mode, int32_t nrep, const mpx_accept_store_batch* b,
                                        uint8_t* out, uint64_t out_cap, uint64_t* dest_off,
                                        void* work, uint64_t work_bytes, uint32_t* err,
                                        hipStream_t stream) {
    if (nrep < 1 || nrep > MPX_MAX_REPLICAS) return hipErrorInvalidValue;
    if (mode != MPX_MODE_MIN) {  // no log on CLASSIC's wire: the dense encoder's frames
        mpx_accept_batch d{};
        d.sends = b->sends;
        d.n_sends = b->n_sends;
        d.inst_base = b->inst_base;
        d.ipg = b->ipg;
        d.n_groups = b->n_groups;
        d.groups = b->groups;
        d.peer_commits = b->peer_commits;
        d.cmd_op = b->cmd_op;
        d.cmd_key = b->cmd_key;
        d.cmd_val = b->cmd_val;
        d.n_cmds = b->n_cmds;
        d.flags = b->flags;
        d.alive_mask = b->alive_mask;
        return launch_encode_accepts(mode, nrep, &d, out, out_cap, dest_off, work, work_bytes, err,
                                     stream);
    }
    const uint64_t n_inst = (uint64_t)b->n_groups * b->ipg;
    const uint64_t items = (uint64_t)nrep * b->n_sends;
    if (b->n_sends >= (1ull << 32) || n_inst > (1ull << 32)) return hipErrorInvalidValue;
    if (items == 0) {
        k_zero_u64<<<1, 64, 0, stream>>>(dest_off, (uint32_t)nrep + 1);
        return hipGetLastError();
    }
    Carver c(work);
    const CatchupWork w(c, (uint32_t)nrep, b->n_sends, n_inst, true);
    if (work_bytes < c.bytes()) return hipErrorInvalidValue;
    const AsArgs a{{b->sends, b->n_sends, b->inst_base, b->ipg, n_inst, b->groups, b->peer_commits,
                    b->cmd_op, b->cmd_key, b->cmd_val},
                   {b->st, b->lb, b->inst, b->src_op, b->src_key, b->src_val, b->n_src, w.lcoff},
                   w.log_off,
                   (uint32_t)nrep,
                   (b->flags & MPX_AB_THRIFTY) ? 1u : 0u,
                   b->alive_mask};
    const hipError_t r = store_log_offsets(b->st, b->inst, b->n_src, n_inst, w, stream);
    if (r != hipSuccess) return r;
    return catchup_run(k_as_sizes, k_as_emit, a, w, b->n_sends, items, out, out_cap, dest_off, err,
                       stream);
}

}  // namespace mpx

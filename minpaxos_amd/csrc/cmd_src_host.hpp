// cmd_src_host.hpp — the host side of the command sources (mpx_store_src[], include/mpx.h) that
// store.cpp and record.cpp share: their validation, the host forms' pre-check of an item's commands
// (what assemble.hpp's msg_cmds / send_cmds judge on the device, answered here before any launch,
// so the two must agree on which batch is legal) and their staging. Internal: nothing here is ABI.
#pragma once
#include <string>

#include "engine_host.hpp"

namespace mpx_host {

// what both forms check of every source; recs: the records they hold
inline int src_args(mpx_engine* e, const mpx_store_src* src, size_t n_src, uint64_t* recs) {
    *recs = 0;
    for (size_t s = 0; s < n_src; ++s) {
        const mpx_store_src& x = src[s];
        if ((x.n_cmds && (!x.op || !x.key || !x.val)) || (x.n_frames && !x.cmd_off))
            return fail(e, MPX_E_INVAL, "null argument");
        *recs += x.n_recs;
    }
    return MPX_OK;
}

// record p of the merged batch lies in the first source whose rec_end is above p
struct SrcIndex {
    const mpx_store_src* src;
    size_t n_src;
    uint64_t rec_end[MPX_SC_MAX_SRC], recs = 0;
    SrcIndex(const mpx_store_src* src_, size_t n) : src(src_), n_src(n) {
        for (size_t s = 0; s < n; ++s) rec_end[s] = recs += src[s].n_recs;
    }
    const mpx_store_src& of(uint64_t p) const {
        size_t s = 0;
        while (s + 1 < n_src && p >= rec_end[s]) ++s;
        return src[s];
    }
};

inline int perm_args(mpx_engine* e, const SrcIndex& idx, const uint32_t* perm, size_t n) {
    if (perm)
        for (size_t i = 0; i < n; ++i)
            if (perm[i] >= idx.recs) return fail(e, MPX_E_INVAL, "a perm entry is out of range");
    return MPX_OK;
}

// The commands of a message item whose record is p (perm[i], or i without perm) and of an
// mpx_accept_send: *len of them, or the code the call answers. what: "storing" / "recording".
inline int resolve_msg(mpx_engine* e, const SrcIndex& idx, uint64_t p, uint32_t value_id, const char* what,
                       uint64_t* len) {
    const mpx_store_src& x = idx.of(p);
    if (value_id >= x.n_frames)
        return fail(e, MPX_E_INVAL, std::string("a ") + what + " item's value_id is not a frame of its source");
    const uint64_t lo = x.cmd_off[value_id], hi = x.cmd_off[value_id + 1];
    if (hi < lo) return fail(e, MPX_E_INVAL, "cmd_off decreases");
    if (hi > x.n_cmds || hi - lo >= 0xFFFFFFFFull)
        return fail(e, MPX_E_INVAL, std::string("a ") + what + " item's command range leaves [0, n_cmds)");
    *len = hi - lo;
    return MPX_OK;
}
inline int resolve_send(mpx_engine* e, const mpx_store_src& src0, const mpx_accept_send& x, const char* what,
                        uint64_t* len) {
    if (x.first_cmd > src0.n_cmds || x.n_cmds > src0.n_cmds - x.first_cmd || x.n_cmds == 0xFFFFFFFFu)
        return fail(e, MPX_E_INVAL, std::string("a ") + what + " item's command range leaves [0, n_cmds)");
    *len = x.n_cmds;
    return MPX_OK;
}

// The sources' arrays in a host form's Stage: four slots per source, add()ed by the constructor;
// after the Stage's commit(), in() copies them in and dev() is the device-side mpx_store_src[]
// (an empty array keeps its null pointer).
class StagedSrcs {
  public:
    StagedSrcs(Stage& L, const mpx_store_src* src, size_t n_src) : L_(L), src_(src), n_(n_src) {
        for (size_t s = 0; s < n_; ++s) {
            const mpx_store_src& x = src_[s];
            slot_[s][0] = L_.add(x.n_frames ? (x.n_frames + 1) * sizeof(uint64_t) : 0);
            slot_[s][1] = L_.add(x.n_cmds);
            slot_[s][2] = L_.add(x.n_cmds * sizeof(int64_t));
            slot_[s][3] = L_.add(x.n_cmds * sizeof(int64_t));
        }
    }
    int in() {
        for (size_t s = 0; s < n_; ++s) {
            const mpx_store_src& x = src_[s];
            const void* const h[4] = {x.cmd_off, x.op, x.key, x.val};
            for (int k = 0; k < 4; ++k) CK(L_.in(slot_[s][k], h[k]));
            d_[s] = x;
            d_[s].cmd_off = L_.at<uint64_t>(slot_[s][0], x.n_frames ? x.cmd_off : nullptr);
            d_[s].op = L_.at<uint8_t>(slot_[s][1], x.n_cmds ? x.op : nullptr);
            d_[s].key = L_.at<int64_t>(slot_[s][2], x.n_cmds ? x.key : nullptr);
            d_[s].val = L_.at<int64_t>(slot_[s][3], x.n_cmds ? x.val : nullptr);
        }
        return MPX_OK;
    }
    const mpx_store_src* dev() const { return d_; }

  private:
    Stage& L_;
    const mpx_store_src* src_;
    size_t n_;
    Slot slot_[MPX_SC_MAX_SRC][4];
    mpx_store_src d_[MPX_SC_MAX_SRC];
};

}  // namespace mpx_host

// engine_host.hpp — the host side's private parts that more than one translation unit of the
// C-ABI layer needs (engine.cpp, order.cpp, client.cpp, replies.cpp, execute.cpp, store.cpp, record.cpp,
// accepts_stored.cpp, prepare_handle.cpp): the handle,
// error reporting, the families' scratch buffers and the staging arena of the host-pointer forms.
// The command sources of store.cpp and record.cpp (their checks, the pre-check of an item's
// commands, their staging) are cmd_src_host.hpp's, the host side of the kernels' assemble.hpp.
// Internal: nothing here is ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <string>

#include "kernels.hpp"

namespace mpx_host {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

// pinned, GPU-mapped staging of a replica-batch apply: the error word in a 128-byte header, then
// op (cap rounded to 16), key, val, ret (cap each) and conf
struct PinIo {
    uint8_t* p = nullptr;
    size_t cap = 0;  // commands
};

}  // namespace mpx_host

struct mpx_engine {
    int device = 0;
    mpx_config cfg{};
    hipStream_t stream = nullptr;
    std::string err;
    uint32_t* d_err = nullptr;
    unsigned long long* d_red = nullptr;
    uint32_t* d_tctl = nullptr;  // tile kernels' control words (kTileCtlWords, zero between calls)
    // host-API staging: one arena, laid out afresh by every host-pointer call (Stage); it grows
    // to the largest single call
    mpx_host::DevBuf arena;
    // global KV table (mpx_apply)
    mpx::KvTable kv{};
    bool kv_ready = false;
    // the families' scratch: grown by the host forms and the *_reserve calls, never by a _dev form
    mpx_host::DevBuf apply_work, decode_work, stream_work, fan_work, log_work, replay_work,
        are_work, ab_work, um_work, cm_work, ord_work, cl_work, rp_work, xg_work, st_work, lr_work,
        pr_work;
    size_t um_var_cap = 0, um_log_cap = 0;  // what um_work was last sized for (mpx_unmarshal_frames)
    size_t cm_send_cap = 0, cm_other_cap = 0;  // ... and cm_work (mpx_encode_commits_reserve)
    size_t xg_inst_cap = 0, xg_group_cap = 0;  // ... and xg_work (mpx_execute_gather_reserve)
    mpx::ApplyOpts apply{};  // mpx_config.apply_* (fixed for the handle's life)
    // replica-sized mpx_apply calls: pinned, GPU-mapped staging the one-launch kernel reads the
    // commands from and writes the results to (no DMA copies on the call's path)
    mpx_host::PinIo pin_io;       // mpx_apply's (copies in and out)
    mpx_host::PinIo pin_staged;   // mpx_apply_buffers / mpx_apply_staged's (the caller fills it)
    // group-step work list (groups the fast kernel hands to the general kernel) + its count
    mpx_host::DevBuf worklist;
    uint32_t* d_wcount = nullptr;
    hipEvent_t ev_fast0 = nullptr, ev_fast1 = nullptr;  // mpx_group_step_events
    bool slots_dirty = false;  // a one-launch fold timed out: zero the packed slots first
    // RCCL
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
};

namespace mpx_host {

inline int fail(mpx_engine* e, int code, const std::string& what) {
    if (e) e->err = what;
    return code;
}

inline int hip_fail(mpx_engine* e, const char* what, hipError_t r) {
    return fail(e, MPX_E_HIP, std::string(what) + ": " + hipGetErrorString(r));
}

#define HIPCHK(e, x)                                        \
    do {                                                    \
        hipError_t _r = (x);                                \
        if (_r != hipSuccess) return hip_fail((e), #x, _r); \
    } while (0)

inline int grow(mpx_engine* e, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return MPX_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    size_t c = std::max(bytes, (size_t)256);
    if (hipMalloc(&b.p, c) != hipSuccess) {
        (void)hipGetLastError();
        return fail(e, MPX_E_NOMEM, "device allocation of " + std::to_string(c) + " bytes failed");
    }
    b.cap = c;
    return MPX_OK;
}

#define GROW(e, buf, bytes)                       \
    do {                                          \
        int _c = grow((e), (buf), (bytes));       \
        if (_c) return _c;                        \
    } while (0)

inline hipStream_t pick(mpx_engine* e, void* s) { return s ? (hipStream_t)s : e->stream; }

inline int check_errword(mpx_engine* e, uint32_t w) {
    if (!w) return MPX_OK;
    // a one-launch step's fold gave up on its slots: zero them before the next step (stream
    // order), so no straggler's late add carries into a later step's totals
    if (w & mpx::kErrSlots) e->slots_dirty = true;
    if (w & mpx::kErrNil)
        return fail(e, MPX_E_NIL_INSTANCE, "record names a nil or out-of-window instance");
    if (w & mpx::kErrBadId) return fail(e, MPX_E_BAD_ID, "reply id outside [0, N)");
    if (w & mpx::kErrOrder)
        return fail(e, MPX_E_INVAL, "records are not grouped in ascending instance order");
    if (w & mpx::kErrKvFull) return fail(e, MPX_E_KV_FULL, "KV table capacity exceeded");
    return fail(e, MPX_E_INVAL, "malformed input (offsets / sizes)");
}

// synchronise the engine stream, read and clear the device error word
inline int finish(mpx_engine* e) {
    uint32_t w = 0;
    HIPCHK(e, hipMemcpyAsync(&w, e->d_err, sizeof(w), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (w) HIPCHK(e, hipMemsetAsync(e->d_err, 0, sizeof(uint32_t), e->stream));
    return check_errword(e, w);
}

inline int begin(mpx_engine* e) {
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemsetAsync(e->d_err, 0, sizeof(uint32_t), e->stream));
    return MPX_OK;
}

inline int h2d(mpx_engine* e, void* d, const void* h, size_t bytes) {
    if (!bytes) return MPX_OK;
    HIPCHK(e, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, e->stream));
    return MPX_OK;
}
inline int d2h(mpx_engine* e, void* h, const void* d, size_t bytes) {
    if (!bytes) return MPX_OK;
    HIPCHK(e, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, e->stream));
    return MPX_OK;
}
#define CK(x)                  \
    do {                       \
        int _c = (x);          \
        if (_c) return _c;     \
    } while (0)

// One host-pointer call's layout of the staging arena. add() names the call's slots at
// 256-byte-aligned offsets (so every slot keeps the 16-byte alignment the tile kernels' vector
// loads need); commit() grows the arena once, to the sum; in() / out() / at() resolve a slot
// against the grown arena, so they are valid only after commit() and no pointer survives a grow.
// An optional array the caller did not pass gets a 0-byte slot and at(slot, nullptr) == nullptr.
struct Slot {
    size_t off, bytes;
};
class Stage {
  public:
    explicit Stage(mpx_engine* e) : e_(e) {}
    Slot add(size_t bytes) {
        const Slot s{end_, bytes};
        end_ += (bytes + 255) & ~(size_t)255;
        return s;
    }
    int commit() {
        CK(grow(e_, e_->arena, std::max(end_, (size_t)1)));  // (never a null base)
        base_ = (char*)e_->arena.p;
        return MPX_OK;
    }
    template <typename T>
    T* at(Slot s) const {
        return reinterpret_cast<T*>(base_ + s.off);
    }
    template <typename T>
    T* at(Slot s, const void* asked) const {
        return asked ? at<T>(s) : nullptr;
    }
    int in(Slot s, const void* h) const { return h2d(e_, base_ + s.off, h, s.bytes); }
    int out(Slot s, void* h) const { return d2h(e_, h, base_ + s.off, s.bytes); }
    int out(Slot s, void* h, size_t bytes) const { return d2h(e_, h, base_ + s.off, bytes); }

  private:
    mpx_engine* e_;
    size_t end_ = 0;
    char* base_ = nullptr;
};

// the body of every *_reserve call: grow a family's scratch so its _dev form can run
inline int reserve(mpx_engine* e, DevBuf& work, uint64_t bytes) {
    CK(begin(e));
    GROW(e, work, bytes);
    return finish(e);
}
// ... and the _dev form's side of it: the scratch must already hold `need` bytes
inline int reserved(mpx_engine* e, const DevBuf& work, uint64_t need, const char* entry,
                    const char* reserve_call) {
    if (work.cap >= need) return MPX_OK;
    return fail(e, MPX_E_INVAL, std::string(entry) + ": call " + reserve_call +
                                    " first (the dev entry point never allocates)");
}

// ---- what the two forms of the Accept encoder share (engine.cpp, accepts_stored.cpp) ----------
inline int propose_shape(mpx_engine* e, size_t n_groups, size_t n_inst, uint32_t ipg) {
    if (n_groups > (1ull << 32) || n_inst > (1ull << 32) ||
        (n_groups ? (!ipg || n_groups * (uint64_t)ipg != n_inst) : n_inst != 0))
        return fail(e, MPX_E_INVAL, "n_inst must equal n_groups * ipg (at most 2^32)");
    return MPX_OK;
}

// bcastAccept's ring walk from self (bareminpaxos.go:465-482 / paxos.go:312-327): bit q set when
// q receives the Accept
inline uint32_t accept_dests(int mode, int32_t N, int32_t self, bool thrifty, uint32_t alive) {
    const int n = thrifty ? N >> 1 : N - 1;
    uint32_t m = 0;
    int32_t q = self;
    for (int sent = 0; sent < n;) {
        q = (q + 1) % N;
        if (q == self) break;
        if (mode != MPX_MODE_MIN && !((alive >> q) & 1u)) continue;
        ++sent;
        m |= 1u << q;
    }
    return m;
}

}  // namespace mpx_host
